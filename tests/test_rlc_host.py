"""CPU suite of the random linear combination (include/handel_gpu.h:
hg_verify_aggregate_rlc and its companions): the coefficients by the code the
device runs (hg_debug_rlc_coeffs) against a hashlib restatement, the mapping's
replacement of 0 by 1 in a host-compiled unit (tests/native/rlc_host.cpp), the
argument errors, the ABI surface, and the register and LDS budgets of the two
GT stages. No GPU needed."""

import ctypes
import hashlib
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
LIB = os.path.join(ROOT, "handel_amd", "_build", "libhandel_gpu.so")

NEW_SYMBOLS = ("hg_verify_aggregate_rlc", "hg_verify_aggregate_rlc_device", "hg_rlc_stats", "hg_debug_rlc_coeffs",
               "hg_debug_rlc_g1", "hg_debug_rlc_groups")
HG_OK, HG_ERR_ARG = 0, 100
SEEDS = (bytes(range(32)), hashlib.sha256(b"rlc-host-seed").digest())


def _lib():
    from handel_amd import _lib as B

    return B.load()


def want_coeff(seed: bytes, i: int) -> int:
    r = int.from_bytes(hashlib.sha256(b"hg-rlc-v1" + seed + i.to_bytes(8, "little")).digest()[:8], "little")
    return r or 1


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("first", [0, 1, 2**32 - 1, 2**32])
def test_coefficients_match_hashlib(seed, first):
    L = _lib()
    out = (ctypes.c_uint64 * 64)()
    assert L.hg_debug_rlc_coeffs(seed, first, 64, out) == HG_OK
    assert [int(v) for v in out] == [want_coeff(seed, first + j) for j in range(64)]


def test_coefficients_differ_by_seed_and_index():
    L = _lib()
    a, b = (ctypes.c_uint64 * 64)(), (ctypes.c_uint64 * 64)()
    assert L.hg_debug_rlc_coeffs(SEEDS[0], 0, 64, a) == HG_OK and L.hg_debug_rlc_coeffs(SEEDS[1], 0, 64, b) == HG_OK
    assert len(set(a)) == 64 and not set(a) & set(b) and 0 not in set(a) | set(b)


def test_engine_wrapper_gives_the_same_coefficients():
    from handel_amd.engine import Engine

    got = Engine.debug_rlc_coeffs(SEEDS[1], 2**32 - 3, 7)
    assert [int(v) for v in got] == [want_coeff(SEEDS[1], 2**32 - 3 + j) for j in range(7)]


def test_zero_maps_to_one_in_the_host_compiled_unit(tmp_path):
    exe = str(tmp_path / "rlc_host")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror",
                           "-Wno-unknown-pragmas",  # hg_sha256.h's unroll hints are the device compiler's
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "handel_amd", "csrc"),
                           os.path.join(ROOT, "tests", "native", "rlc_host.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    assert r.stderr == "", r.stderr[-2000:]  # no sanitizer report
    assert r.stdout == "ok\n"


def test_argument_errors_without_gpu():
    L = _lib()
    seed = SEEDS[0]
    buf = ctypes.create_string_buffer(256)
    # a context that is never read: the seed and the group are checked first
    ctx = ctypes.cast(ctypes.create_string_buffer(64), ctypes.c_void_p)
    for fn, args in (
        (L.hg_verify_aggregate_rlc, lambda c, sd, g: (c, buf, 1, buf, 1, buf, sd, g, buf)),
        (L.hg_verify_aggregate_rlc_device, lambda c, sd, g: (c, buf, 1, buf, buf, sd, g, buf, None)),
    ):
        assert fn(*args(ctx, seed, 0)) == HG_ERR_ARG        # group == 0
        assert fn(*args(ctx, seed, 4097)) == HG_ERR_ARG     # group > 4096
        assert fn(*args(ctx, None, 64)) == HG_ERR_ARG       # NULL seed
        assert fn(*args(None, seed, 64)) == HG_ERR_ARG      # NULL context
    assert L.hg_debug_rlc_g1(ctx, buf, 1, buf, 0, buf) == HG_ERR_ARG
    assert L.hg_debug_rlc_g1(ctx, buf, 1, buf, 4097, buf) == HG_ERR_ARG
    assert L.hg_debug_rlc_g1(None, buf, 1, buf, 3, buf) == HG_ERR_ARG
    assert L.hg_debug_rlc_groups(ctx, buf, 1, buf, 1, buf, buf, 0, buf, buf, buf) == HG_ERR_ARG
    assert L.hg_debug_rlc_groups(None, buf, 1, buf, 1, buf, buf, 3, buf, buf, buf) == HG_ERR_ARG
    assert L.hg_rlc_stats(None, None, None, None) == HG_ERR_ARG
    assert L.hg_debug_rlc_coeffs(None, 0, 1, buf) == HG_ERR_ARG
    assert L.hg_debug_rlc_coeffs(seed, 0, 1, None) == HG_ERR_ARG
    assert L.hg_debug_rlc_coeffs(seed, 0, 0, None) == HG_OK


def test_header_declares_and_library_exports_the_entry_points():
    from handel_amd import _lib as B

    header = open(os.path.join(ROOT, "include", "handel_gpu.h")).read()
    L = _lib()
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert hasattr(L, name) and name in B.SIGNATURES, name


def test_go_and_integration_mirror_the_entry_points():
    go = open(os.path.join(ROOT, "go", "bn256", "hip", "engine.go")).read()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in ("hg_verify_aggregate_rlc", "hg_verify_aggregate_rlc_device"):
        assert name in go and name in doc, name
    assert "crypto/rand" in go


# ---------------------------------------------------------------- kernel resources
# the two GT stages run in the FOLD team region, five 12-lane teams a wave
# (12000 bytes of LDS), inside the fold kernels' budget of two waves per SIMD
# (at most 256 VGPRs), without scratch
STAGES = ("k_rlc_subsets", "k_rlc_horner")
OTHERS = ("k_rlc_prep", "k_rlc_g1_mul", "k_rlc_g1_sum", "k_rlc_count", "k_rlc_bcount", "k_rlc_scan", "k_rlc_gather",
          "k_rlc_scatter")


@pytest.fixture(scope="module")
def res():
    if not os.path.exists(LIB):
        pytest.skip("libhandel_gpu.so not built")
    import kernel_sizes

    r = kernel_sizes.resources(LIB)
    if not r:
        pytest.skip("no gfx950 code object metadata found")
    return r


def _one(res, part):
    hits = {k: v for k, v in res.items() if part in k}
    assert len(hits) == 1, (part, sorted(hits))
    return next(iter(hits.values()))


@pytest.mark.parametrize("part", STAGES + OTHERS)
def test_kernels_keep_their_budgets(res, part):
    r = _one(res, part)
    assert r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0 and r["scratch"] == 0, (part, r)
    if part in STAGES:
        assert r["lds"] == 12000 and r["vgpr"] <= 256, (part, r)
