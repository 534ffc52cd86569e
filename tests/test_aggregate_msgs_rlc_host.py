"""CPU suite of the per-message random linear combination (include/handel_gpu.h:
hg_verify_aggregate_msgs_rlc and its companions): the ABI
surface, the argument errors, the mod-Order scaling of hashedMessage's scalar in
a host-compiled unit (tests/native/mrlc_scale.cpp, under the address and
undefined-behaviour sanitizers) against Python integers, and the register and
LDS budgets of the new kernels. No GPU needed."""

import ctypes
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
LIB = os.path.join(ROOT, "handel_amd", "_build", "libhandel_gpu.so")

NEW_SYMBOLS = ("hg_verify_aggregate_msgs_rlc", "hg_verify_aggregate_msgs_rlc_device", "hg_verify_multisig_msgs_rlc",
               "hg_debug_msgs_rlc_groups", "hg_debug_msgs_rlc_points")
HG_OK, HG_ERR_ARG = 0, 100
ORDER = 65000549695646603732796438742359905742570406053903786389881062969044166799969


def _lib():
    from handel_amd import _lib as B

    return B.load()


def test_header_declares_and_library_exports_the_entry_points():
    from handel_amd import _lib as B

    header = open(os.path.join(ROOT, "include", "handel_gpu.h")).read()
    L = _lib()
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert hasattr(L, name) and name in B.SIGNATURES, name


def test_go_and_integration_mirror_the_verify_calls():
    go = open(os.path.join(ROOT, "go", "bn256", "hip", "engine.go")).read()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in ("hg_verify_aggregate_msgs_rlc_device", "hg_verify_multisig_msgs_rlc"):
        assert re.search(r"C\.%s\(" % name, go), name
        assert name in doc, name
    assert "hg_verify_aggregate_msgs_rlc(" in doc and "crypto/rand" in go


def test_argument_errors_without_gpu():
    L = _lib()
    seed = bytes(range(32))
    buf = ctypes.create_string_buffer(256)
    # a context that is never read: the seed and the group are checked first
    ctx = ctypes.cast(ctypes.create_string_buffer(64), ctypes.c_void_p)
    for fn, args in (
        (L.hg_verify_aggregate_msgs_rlc, lambda c, sd, g: (c, buf, 1, buf, buf, buf, 1, buf, 1, buf, sd, g, buf)),
        (L.hg_verify_aggregate_msgs_rlc_device,
         lambda c, sd, g: (c, buf, 1, buf, buf, buf, 1, buf, buf, sd, g, buf, None)),
        (L.hg_verify_multisig_msgs_rlc, lambda c, sd, g: (c, buf, 1, buf, buf, buf, buf, 1, buf, 1, buf, sd, g, buf)),
    ):
        assert fn(*args(ctx, seed, 0)) == HG_ERR_ARG        # group == 0
        assert fn(*args(ctx, seed, 4097)) == HG_ERR_ARG     # group > 4096
        assert fn(*args(ctx, None, 64)) == HG_ERR_ARG       # NULL seed
        assert fn(*args(None, seed, 64)) == HG_ERR_ARG      # NULL context
    groups = lambda c, g: (c, buf, 1, buf, buf, buf, 1, buf, 1, buf, buf, g, buf, buf, buf)  # noqa: E731
    assert L.hg_debug_msgs_rlc_groups(*groups(ctx, 0)) == HG_ERR_ARG
    assert L.hg_debug_msgs_rlc_groups(*groups(ctx, 4097)) == HG_ERR_ARG
    assert L.hg_debug_msgs_rlc_groups(*groups(None, 3)) == HG_ERR_ARG
    assert L.hg_debug_msgs_rlc_points(None, buf, 1, buf, buf, buf, 1, buf) == HG_ERR_ARG
    assert L.hg_debug_msgs_rlc_points(ctx, buf, 1, buf, buf, None, 1, buf) == HG_ERR_ARG
    assert L.hg_debug_msgs_rlc_points(ctx, None, 0, None, None, None, 0, None) == HG_OK  # n == 0: nothing read


# ---------------------------------------------------------------- k' = r k mod Order
def test_scaling_matches_python_integers(tmp_path):
    exe = str(tmp_path / "mrlc_scale")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror",
                           "-Wno-unknown-pragmas",  # the unroll hints are the device compiler's
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "handel_amd", "csrc"),
                           os.path.join(ROOT, "tests", "native", "mrlc_scale.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    assert r.stderr == "", r.stderr[-2000:]  # no sanitizer report
    rows = [tuple(int(x, 16) for x in line.split()) for line in r.stdout.splitlines()]
    assert len(rows) == 48 and all(len(row) == 3 for row in rows)
    for rr, k, got in rows:
        assert got == rr * k % ORDER, (hex(rr), hex(k), hex(got))
    pairs = {(rr, k) for rr, k, _ in rows}
    rs, ks = {rr for rr, _ in pairs}, {k for _, k in pairs}
    assert {1, 2**64 - 1} <= rs and {0, ORDER - 1} <= ks
    # products just above a multiple of Order, small and large quotients
    near = [(rr, k) for rr, k in pairs if k < ORDER and rr * k > ORDER and rr * k % ORDER < 2**64]
    assert {rr * k // ORDER for rr, k in near} >= {2, 2**63, 12345678901234567}
    assert any(rr * k % ORDER == 1 for rr, k in near)
    assert any(k >= ORDER for k in ks)  # reduced first


# ---------------------------------------------------------------- kernel resources
# k_mrlc_miller is k_verify_ml<4>'s body (layout V: 20480 bytes of LDS, two
# waves per SIMD); k_mrlc_product runs in the FOLD team region, five 12-lane
# teams a wave (12000 bytes)
BUDGETS = {"k_mrlc_miller": 20480, "k_mrlc_product": 12000}
OTHERS = ("k_mrlc_scalars", "k_mrlc_sigs", "k_mrlc_carrier", "k_mrlc_checks", "k_mrlc_gather")


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


@pytest.mark.parametrize("part", tuple(BUDGETS) + OTHERS)
def test_kernels_keep_their_budgets(res, part):
    r = _one(res, part)
    assert r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0 and r["scratch"] == 0, (part, r)
    if part in BUDGETS:
        assert r["lds"] == BUDGETS[part] and r["vgpr"] <= 256, (part, r)


def test_every_new_kernel_is_listed(res):
    names = {k for k in res if "k_mrlc_" in k}
    assert len(names) == len(BUDGETS) + len(OTHERS), sorted(names)
    for k in names:
        r = res[k]
        assert r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0 and r["scratch"] == 0, (k, r)
